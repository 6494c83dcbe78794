"""GPU: model.decoder_rows under data parallelism -- the two-process set-up of tests/dp_worker.py (RCCL with two GPUs, gloo with
both ranks on cuda:0 otherwise) on a model with the option on: the reduced gradients equal the single-process ones, the bound
of test_two_rank_data_parallel_equivalence_on_the_hip_engine (1e-5 relative Frobenius, losses 1e-6)."""
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


def test_two_rank_data_parallel_with_decoder_rows(tmp_path):
    world = 2
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    out_file = str(tmp_path / "dp_decoder_rows.pt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "dp_decoder_rows_worker.py"), out_file, "backward", "tiny"],
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
    got = torch.load(out_file)
    assert got["ranks_agree"] and got["world"] == 2 and got["covers"] and got["collectives"] >= 3
    # the single-process reference with the option on: the same four samples, two per step, DDP loss convention
    cfg = _tiny_cfg()
    m = build(cfg, O.synth_params(cfg, seed=41, std=0.05, ln_jitter=0.1))
    m.decoder_rows = True
    batch = synth_batch(cfg, B=4, L=60, seed=9)
    m.zero_grad(set_to_none=False)
    losses = []
    for r in range(2):
        out = m(**{k: v[2 * r:2 * r + 2].to(DEV) for k, v in batch.items()})
        assert out._run.dec_plan is not None
        out.loss.backward()
        losses.append(out.loss.item())
    want = {n: p.grad.float().cpu() / 2 for n, p in m.named_parameters() if p.requires_grad}
    assert abs(got["losses"][0] - losses[0]) < 1e-6 and abs(got["losses"][1] - losses[0]) < 1e-6
    worst = max(_rel_fro(got["grads"][n], want[n]) for n in want)
    print(f"[dp decoder_rows] worst relative difference reduced-vs-single-process: {worst:.2e}")
    assert worst < 1e-5, worst
