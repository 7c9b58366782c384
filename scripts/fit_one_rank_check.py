#!/usr/bin/env python
"""One epoch of ptt_amd.fit.fit on a ONE-rank `nccl` (= RCCL) process group with force_ddp=True: the captured step is then two
hipGraphs around the eager all-reduce, and the step ledger's append is recorded in the SECOND one, behind the optimizer's update.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port P scripts/fit_one_rank_check.py

Prints one JSON line: the ledger's rows as float32 bit patterns, a SHA-256 digest of the final model and optimizer state, and
what the trainer captured. tests/test_fit_gpu.py compares it with the same epoch run in its own process without a group
(`one_epoch(dev, force_ddp=False)`): with one participant the all-reduce is an identity, so everything must be equal."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def state_digest(trainer):
    """SHA-256 over the tracker's state_dict and the optimizer's state tensors, in their own order."""
    h = hashlib.sha256()
    for k, v in trainer.tracker.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    state = trainer.optimizer.state_dict()['state']
    for k in sorted(state):
        for name in sorted(state[k]):
            h.update(("%s.%s" % (k, name)).encode())
            h.update(torch.as_tensor(state[k][name]).detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def one_epoch(dev, force_ddp):
    from ptt_amd import synth
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.fit import StepLedger, fit
    from ptt_amd.models import build_network
    from ptt_amd.train_feed import TrainBatchFeeder
    from ptt_amd.train_step import DataParallelTrainer
    tracklets = [synth.tracklet(seed, 6, n_obj=(100, 300), n_bg=(300, 800)) for seed in range(4)]
    feeder = TrainBatchFeeder(tracklets, dev, batch_size=4, spare=2, candidates_per_frame=1, seed=5)
    torch.manual_seed(1)
    model = build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev).train()
    trainer = DataParallelTrainer(model, dev, graph=True, force_ddp=force_ddp, ledger=StepLedger(dev, capacity=16))
    with tempfile.TemporaryDirectory() as ckpt_dir:
        records = fit(trainer, feeder, 1, ckpt_dir)
    torch.cuda.synchronize()
    rows = trainer.ledger.ring[:len(feeder)].cpu().numpy()
    cap = trainer.captured
    return {"rows_bits": rows.view(np.int32).tolist(), "digest": state_digest(trainer), "steps": records[0]["steps"],
            "non_finite": records[0]["non_finite"], "mean_loss": records[0]["loss"], "graph_steps": trainer.graph_steps,
            "two_graphs": cap is not None and cap.second is not None, "ledger_in_graph": cap is not None and bool(cap.ledger),
            "collective": bool(trainer.collective), "ledger_fed": bool(trainer.ledger_fed)}


def main():
    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29543")
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    one = torch.ones(1, device=dev)
    dist.all_reduce(one)
    out = one_epoch(dev, force_ddp=True)
    out.update(world=world, ranks_seen=int(one.item()), backend=dist.get_backend())
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
