"""One rank of the two-rank check of the fine-tuning launch graphs (launched by tests/test_gpu_finetune_graphs.py).

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment; argv[1] = output file (rank 0 writes it).

`model.finetune_graphs` is on on both ranks; rank 1's capture budget is used up before its first step, so it switches the
feature off by itself and serves every step eagerly while rank 0 replays its graphs.  Both must issue the same collectives
(one all-reduce over the whole flat gradient buffer per step: the reducer stays in "after" placement on the rank that fell
back) and end with the same reduced gradients.  Backend as in tests/dp_worker.py: nccl with one GPU per rank when the box
has two, gloo with both ranks on cuda:0 otherwise.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

N_ANS, L_TEXT = 40, 32


def make_model():
    """the tiny downstream model (dropout off, so ranks and the single process draw nothing) in training mode"""
    from tests.test_gpu_downstream import hip_model

    a2tok = torch.randint(1, 300, (N_ANS, 3), generator=torch.Generator().manual_seed(17))
    cfg, _, m = hip_model(N_ANS, 10, a2tok, train=True)
    return cfg, m


def make_inputs(cfg, rank, per, dev):
    """shard `rank` of a ragged batch of 2 * per samples, one requested row inside every sample's text, an answer each"""
    from tests.golden.make_goldens import synth_batch

    b = synth_batch(cfg, B=2 * per, L=L_TEXT, seed=9)
    b.pop("labels")
    ans = torch.randint(0, N_ANS, (2 * per,), generator=torch.Generator().manual_seed(9))
    mine = {k: v[rank * per:(rank + 1) * per].to(dev) for k, v in b.items()}
    tlen = mine["attention_mask"].sum(1)
    rows = torch.arange(per, device=dev) * (cfg.max_feats + L_TEXT) + cfg.max_feats + tlen // 2
    return mine, rows, ans[rank * per:(rank + 1) * per].to(dev)


def main():
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    multi = torch.cuda.device_count() >= world
    dev = torch.device("cuda", rank if multi else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl" if multi else "gloo", init_method="env://", world_size=world, rank=rank)

    import frozenbilm_amd.train_graph as TG
    from frozenbilm_amd.parallel import GradReducer

    cfg, m = make_model()
    m.to(dev)
    m.train()
    m.finetune_graphs = True
    if rank == 1:
        TG.MAX_CAPTURES = 0
    red = GradReducer.attach(m, min_bucket_elems=1 << 10, overlap="attention_windows")
    feed, rows, ans = make_inputs(cfg, rank, 2, dev)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (rank 1: the budget warning)
        for _ in range(2):  # two steps: the reducer's bookkeeping must reset between them
            m.zero_grad(set_to_none=False)
            F.cross_entropy(m(logit_rows=rows, **feed)["logits"], ans).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.requires_grad}
    # both ranks: one collective over the whole flat buffer per step, whichever way the step was served
    replays = TG.stats(m, TG.FINETUNE).replays
    mine_pat = torch.tensor([len(red.last_launched), red.last_launched[0][0], red.last_launched[-1][1], red.n_collectives],
                            dtype=torch.int64, device=dev)
    both = [torch.zeros_like(mine_pat) for _ in range(world)]
    dist.all_gather(both, mine_pat)
    pattern_same = (all(torch.equal(both[0], b_) for b_ in both) and int(mine_pat[0]) == 1
                    and (int(mine_pat[1]), int(mine_pat[2])) == (0, red.flat_grad.numel()))
    how = torch.tensor([replays], dtype=torch.int64, device=dev)
    hows = [torch.zeros_like(how) for _ in range(world)]
    dist.all_gather(hows, how)
    print(f"[finetune_graphs_dp_worker] rank {rank}: {replays} replays, finetune_graphs {m.finetune_graphs}, overlap {red.overlap}, "
          f"collectives {[b_.tolist() for b_ in both]}", flush=True)
    assert (replays == 2) == (rank == 0) and m.finetune_graphs is (rank == 0), (rank, replays, m.finetune_graphs)
    flat = torch.cat([g.reshape(-1) for g in grads.values()]).to(dev)
    ref = flat.clone()
    dist.broadcast(ref, src=0)
    ok = torch.tensor([1.0 if torch.equal(ref, flat) else 0.0], device=dev)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if rank == 0:
        torch.save({"grads": grads, "collectives": len(red.last_launched), "overlap": red.overlap, "world": world,
                    "ranks_agree": bool(ok.item() == 1.0), "pattern_same": bool(pattern_same),
                    "served": ["graph" if int(h) else "eager" for h in hows], "replays": [int(h) for h in hows]}, sys.argv[1])
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
