"""One rank of the two-rank data-parallel check of the BERT engine (launched by tests/test_gpu_bert_dp.py).

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment; argv[1] = output file (rank 0 writes it),
    argv[2] = GradReducer.overlap mode, argv[3] = "padded" or "packed" (model.packed_rows).

Backend: nccl (= RCCL) with one GPU per rank when the box has at least WORLD_SIZE GPUs, otherwise gloo with every rank on
cuda:0 -- the same BertEngine / GradReducer code path either way.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

SEED_PARAMS, SEED_BATCH, PER_RANK = 21, 22, 2


def build_model(dev):
    from frozenbilm_amd.model import BertConfig, BertForMaskedLM
    from oracle import bert_oracle as O
    from tests.test_gpu_bert import SMALL, _params

    cfg = O.BertOracleConfig(**SMALL, features_dim=32, max_feats=4)
    m = BertForMaskedLM(BertConfig(**SMALL), features_dim=32, max_feats=4)
    m.load_state_dict(_params(cfg, seed=SEED_PARAMS), strict=False)
    return m.to(dev).eval()  # eval mode: dropout off, gradients on


def shard(rank, dev, world=2):
    from tests.test_gpu_bert import _batch

    batch = _batch(seed=SEED_BATCH, B=PER_RANK * world)  # samples 0 and 2 are ragged: both ranks have rows to drop
    return {k: v[rank * PER_RANK:(rank + 1) * PER_RANK].to(dev) for k, v in batch.items()}


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    out_file, overlap, layout = sys.argv[1], sys.argv[2], sys.argv[3]
    multi = torch.cuda.device_count() >= world
    dev = torch.device("cuda", rank if multi else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl" if multi else "gloo", init_method="env://", world_size=world, rank=rank)

    from frozenbilm_amd.loops import LossLog
    from frozenbilm_amd.parallel import GradReducer

    m = build_model(dev)
    m.packed_rows = layout == "packed"
    # small buckets: the two layer stages and the embeddings leave in collectives of their own where the placement allows it
    red = GradReducer.attach(m, min_bucket_elems=64, overlap=overlap)
    mine = shard(rank, dev, world)
    losses, packed = [], []
    for _ in range(2):  # two steps: the reducer's bookkeeping must reset between them
        m.zero_grad(set_to_none=False)
        out = m(**mine)
        out.loss.backward()  # the engine's backward launches the bucket collectives and joins them (GradReducer.finish)
        losses.append(out.loss.item())
        packed.append(out.__dict__["_run"].pk is not None)
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.requires_grad}
    n_coll, launch_order = len(red.last_launched), list(red.last_launched)
    spans = sorted(red.last_launched)
    covers = spans[0][0] == 0 and spans[-1][1] == red.flat_grad.numel() and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))

    # a third step with the loops' loss bookkeeping: the logged loss rides in front of the first gradient bucket
    class _Meter:
        loss_log = None
        vals = None

        def log(self, **kw):
            self.vals = kw

    meter = _Meter()
    log = LossLog(meter, "mlm_loss", reducer=red)
    m.zero_grad(set_to_none=False)
    out = m(**mine)
    c0 = red.n_collectives
    log.begin(out.loss)
    out.loss.backward()
    log.check()
    extra = red.n_collectives - c0 - len(red.last_launched)
    mean_loss = torch.tensor([out.loss.item()], device=dev)
    dist.all_reduce(mean_loss)
    loss_rides = (red.carries_scalars and meter.vals is not None and abs(meter.vals["loss"] - mean_loss.item() / world) < 1e-6
                  and abs(meter.vals["mlm_loss"] - meter.vals["loss"]) < 1e-12)
    print(f"[bert_dp_worker] rank {rank}/{world}: backend {dist.get_backend()}, overlap {red.overlap}, layout {layout}, "
          f"{n_coll} collectives per step, launch order {launch_order}", flush=True)
    # every rank must hold the same reduced gradients
    flat = torch.cat([g.reshape(-1) for g in grads.values()]).to(dev)
    ref = flat.clone()
    dist.broadcast(ref, src=0)
    ok = torch.tensor([1.0 if torch.equal(ref, flat) else 0.0], device=dev)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    # an engine rebuild (set_answer_embeddings): the reducer follows the model to the new engine's buffers
    old = m.engine()
    m.set_answer_embeddings(torch.randint(1, 300, (5, 2), generator=torch.Generator().manual_seed(3)).to(dev))
    new = m.engine()
    rebound = (new is not old and new.reducer is red and red.flat_grad.data_ptr() == new.flat_grad.data_ptr()
               and red.flat_full is not None and red.flat_full.data_ptr() == new.flat_grad_full.data_ptr()
               and red.bucket_ends == new.bucket_ends)
    m.zero_grad(set_to_none=False)
    m(**mine, mlm=True).loss.backward()  # ... and a step through it still exchanges the whole buffer
    spans2 = sorted(red.last_launched)
    rebound = rebound and spans2[0][0] == 0 and spans2[-1][1] == new.flat_grad.numel()
    torch.cuda.synchronize()
    if rank == 0:
        torch.save({"grads": grads, "losses": losses, "backend": dist.get_backend(), "collectives": n_coll, "overlap": red.overlap,
                    "covers": bool(covers), "launch_order": launch_order, "ranks_agree": bool(ok.item() == 1.0), "world": world,
                    "loss_rides": bool(loss_rides), "extra_collectives_for_the_loss": int(extra), "packed": packed,
                    "rebound": bool(rebound), "stages": sorted(red.bucket_ends)}, out_file)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
