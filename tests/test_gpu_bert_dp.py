"""GPU: data-parallel gradient exchange of the BERT variant (parallel.GradReducer on bert_engine.BertEngine): two processes, one
rank each, over RCCL when the box has two GPUs and over gloo with both ranks on cuda:0 otherwise (tests/bert_dp_worker.py)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run_two_ranks(tmp_path, overlap, layout):
    world = 2
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    out_file = str(tmp_path / f"bert_dp_{overlap}_{layout}.pt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "bert_dp_worker.py"), out_file, overlap, layout],
                                      env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p_ in procs:
        try:
            o, _ = p_.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p_.kill()
            o, _ = p_.communicate()
        logs.append(o)
    assert all(p_.returncode == 0 for p_ in procs), "\n".join(logs)
    print("\n".join(l for lg in logs for l in lg.splitlines() if "[bert_dp_worker]" in l))
    return torch.load(out_file)


@pytest.fixture(scope="module")
def single_process():
    """gradients of the same four samples in one process on the padded grid, under the DDP convention (mean over the ranks
    of the per-rank mean loss); computed once for both runs"""
    from tests.bert_dp_worker import build_model, shard

    m = build_model(torch.device(DEV))
    m.zero_grad(set_to_none=False)
    losses = []
    for r in range(2):
        out = m(**shard(r, DEV))
        out.loss.backward()
        losses.append(out.loss.item())
    return {n: p.grad.float().cpu() / 2 for n, p in m.named_parameters() if p.requires_grad}, losses


@pytest.mark.parametrize("overlap,layout", [("backward", "padded"), ("attention_windows", "packed")])
def test_two_rank_data_parallel_on_the_bert_engine(tmp_path, single_process, overlap, layout):
    got = _run_two_ranks(tmp_path, overlap, layout)  # (GradReducer.attach raised NotImplementedError for this model before)
    assert got["world"] == 2 and got["overlap"] == overlap
    assert got["ranks_agree"]                       # both ranks end with identical gradients
    assert got["covers"], got["launch_order"]       # the launched spans cover [0, flat_grad.numel()) without gaps
    assert got["stages"] == ["emb", "layer0", "layer1"]
    assert got["packed"] == [layout == "packed"] * 2
    # the logged loss is the rank mean and travelled with the first bucket: no collective of its own
    assert got["loss_rides"] and got["extra_collectives_for_the_loss"] == 0, got
    if overlap == "backward":  # one collective per stage: layer 1, layer 0, the embeddings
        assert got["collectives"] == 3, got["launch_order"]
    else:  # launched in front of an attention backward (layer 1's bucket in layer 0's window) and at the end
        assert got["collectives"] >= 2, got["launch_order"]
    assert got["rebound"]                           # after an engine rebuild the reducer points at the new engine's buffer
    want, losses = single_process
    assert abs(got["losses"][0] - losses[0]) < 1e-5 and abs(got["losses"][1] - losses[0]) < 1e-5  # rank 0's own loss, both steps
    worst = max((got["grads"][n] - want[n]).norm().item() / (want[n].norm().item() + 1e-12) for n in want)
    print(f"[bert dp {overlap}/{layout}] backend {got['backend']}, {got['collectives']} collectives per step, worst relative "
          f"difference reduced-vs-single-process: {worst:.2e}")
    assert set(got["grads"]) == set(want) and worst < 1e-5, worst
