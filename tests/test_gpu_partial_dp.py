"""GPU: partial fine-tuning under data parallelism -- two ranks on one box (tests/partial_dp_worker.py), only the top layer
live, for each placement of the gradient collectives: the reduced live gradients equal the single-process gradients of the
concatenated batch (1e-5, as tests/test_gpu_model.py holds the full step), the dead slices are zero on every rank, every bucket
leaves (those of stages the backward never reaches at the end of backward), and no rank waits: each process has a time limit."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import deberta_oracle as O  # noqa: E402
from tests.golden.make_goldens import _tiny_cfg, synth_batch  # noqa: E402
from tests.test_gpu_model import _rel_fro, build  # noqa: E402

DEV = "cuda"
LIMIT_S = 150  # per process


def _run_two_ranks(tmp_path, overlap):
    world = 2
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    out_file = str(tmp_path / f"partial_dp_{overlap}.pt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "partial_dp_worker.py"), out_file, overlap],
                                      env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs, timed_out = [], False
    for p_ in procs:
        try:
            o, _ = p_.communicate(timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            timed_out = True
            p_.kill()
            o, _ = p_.communicate()
        logs.append(o)
    assert not timed_out, "a rank waited past its time limit:\n" + "\n".join(logs)
    assert all(p_.returncode == 0 for p_ in procs), "\n".join(logs)
    print("\n".join(l for lg in logs for l in lg.splitlines() if "[partial_dp_worker]" in l))
    return torch.load(out_file)


_REF = {}


def _single_process_reference():
    if not _REF:
        from tests.partial_dp_worker import freeze_below_the_top_layer

        cfg = _tiny_cfg()
        m = build(cfg, O.synth_params(cfg, seed=41, std=0.05, ln_jitter=0.1))
        live = freeze_below_the_top_layer(m)
        batch = synth_batch(cfg, B=4, L=60, seed=9)
        m.zero_grad(set_to_none=False)
        for r in range(2):
            m(**{k: v[2 * r:2 * r + 2].to(DEV) for k, v in batch.items()}).loss.backward()
        named = dict(m.named_parameters())
        _REF.update({n: named[n].grad.float().cpu() / 2 for n in live})
    return _REF


@pytest.mark.parametrize("overlap", ["backward", "attention_windows", "after"])
def test_two_rank_partial_fine_tuning(tmp_path, overlap):
    got = _run_two_ranks(tmp_path, overlap)
    assert got["ranks_agree"] and got["covers"] and got["idle"] and got["overlap"] == overlap, got
    assert got["dead_zero"] and got["dead_have_no_grad"]
    assert got["saved"] == 2  # only the two decoder passes were kept
    want = _single_process_reference()
    assert set(want) == set(got["grads"]) and want
    worst = max(_rel_fro(got["grads"][n], want[n]) for n in want)
    print(f"{overlap}: {got['collectives']} collectives per step; worst relative difference reduced-vs-single-process {worst:.2e}")
    assert worst < 1e-5, worst
