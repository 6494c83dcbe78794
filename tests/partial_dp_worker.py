"""One rank of the two-rank data-parallel check of PARTIAL fine-tuning (launched by tests/test_gpu_partial_dp.py): only the top
layer's parameters are live, on both ranks (the live set must agree across the ranks; that is the caller's duty).

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment; argv[1] = output file (rank 0 writes it),
    argv[2] = GradReducer.overlap mode.  Backend as in tests/dp_worker.py: nccl with one GPU per rank when the box has two, else
    gloo with both ranks on cuda:0.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist


def freeze_below_the_top_layer(m):
    top = f"deberta.encoder.layer.{m.config.num_hidden_layers - 1}."
    live = []
    for n, p in m.named_parameters():
        if n in set(m.trainable_names()):
            p.requires_grad_(n.startswith(top))
            if n.startswith(top):
                live.append(n)
    return live


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    multi = torch.cuda.device_count() >= world
    dev = torch.device("cuda", rank if multi else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl" if multi else "gloo", init_method="env://", world_size=world, rank=rank)

    from frozenbilm_amd.parallel import GradReducer
    from oracle import deberta_oracle as O
    from tests.golden.make_goldens import _tiny_cfg, synth_batch
    from tests.test_gpu_model import build

    cfg = _tiny_cfg()
    m = build(cfg, O.synth_params(cfg, seed=41, std=0.05, ln_jitter=0.1))  # eval mode: dropout off, gradients on
    m.to(dev)
    live = freeze_below_the_top_layer(m)
    red = GradReducer.attach(m, min_bucket_elems=1 << 10, overlap=sys.argv[2])
    per = 2
    batch = synth_batch(cfg, B=per * world, L=60, seed=9)
    mine = {k: v[rank * per:(rank + 1) * per].to(dev) for k, v in batch.items()}
    for _ in range(2):  # two steps: the reducer's bookkeeping must reset between them, also for the buckets no stage signalled
        m.zero_grad(set_to_none=False)
        out = m(**mine)
        saved = len(out._run.layers)
        out.loss.backward()
    torch.cuda.synchronize()
    eng = m.engine()
    named = dict(m.named_parameters())
    grads = {n: named[n].grad.detach().float().cpu() for n in live}
    dead_have_no_grad = all(named[n].grad is None for n in m.trainable_names() if n not in live)
    mk = torch.zeros(eng.flat_grad.numel(), dtype=torch.bool, device=dev)
    for n in live:
        mk[eng.offsets[n]:eng.offsets[n] + named[n].numel()] = True
    dead_zero = not bool(eng.flat_grad[~mk].any())
    spans = sorted(red.last_launched)
    covers = spans[0][0] == 0 and spans[-1][1] == red.flat_grad.numel() and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    idle = not red.pending and not red._ready and not red._done
    print(f"[partial_dp_worker] rank {rank}/{world}: backend {dist.get_backend()}, overlap {red.overlap}, "
          f"{len(red.last_launched)} collectives per step, {saved} layer executions saved", flush=True)
    flat = eng.flat_grad.clone()
    ref = flat.clone()
    dist.broadcast(ref, src=0)
    ok = torch.tensor([1.0 if torch.equal(ref, flat) else 0.0], device=dev)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if rank == 0:
        torch.save({"grads": grads, "covers": covers, "dead_zero": dead_zero, "dead_have_no_grad": dead_have_no_grad, "idle": idle,
                    "ranks_agree": bool(ok.item() == 1.0), "saved": saved, "collectives": len(red.last_launched),
                    "overlap": red.overlap}, sys.argv[1])
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
