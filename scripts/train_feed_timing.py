"""Dev tool: what a training batch costs when ptt_amd.train_feed.TrainBatchFeeder makes it, at B = 48, 1024 / 512, on synthetic
tracklets sized like the reference's pre-cropped KITTI frames (8000 .. 20000 background points per frame):

  (a) the feeder alone, per batch: device time (HIP events the feeder records on its stream right before the upload and right
      after the second launch), host time (the whole call, plan included) and the plan's share of it;
  (b) the same 48 samples through the per-sample functions of ptt_amd.datasets.kitti.kitti_tracking_utils (crop_center_pc with
      labels, get_model, regularize_pc(istrain=True)): wall time per batch, the device drained at the end of it;
  (c) the graphed training step (train_step.DataParallelTrainer) per step: on one resident batch, fed by the feeder on the
      step's own stream, and fed by a feeder with a stream of its own — wall time over the measured steps, same process.

  --augment  instead of (a)-(c): the device time per batch (the events of (a); for the last case up to an event behind the last
      torch op, so the host's gaps between its launches count) of three feeders that take turns batch by batch —
      d_plain                  no augmentor;
      d_augmented              the DATA_AUGMENTOR block of tools/cfgs/kitti_models/p2b.yaml (flip along x, rotation over +-pi/4);
      d_plain_plus_stock_ops   no augmentor, then the same maps applied to search_points / template_points with stock torch ops on
                               the feeder's stream (one small upload, a bmm and a product per cloud): what works without this path.
      The stock-ops variant takes each slot's own map and ignores replacement — it cannot know the source without a read-back.

  --plain-only  instead of (a)-(c): the device time per batch of the feeder without an augmentor alone, one JSON line with the
      library's ABI version and the float64 sum of the last batch's search_points. With --tree DIR the package is imported from
      the checkout DIR (built there) instead of this one: the guard that a commit did not move the default path is this mode run
      in fresh processes against the parent's checkout and this one in turn, e.g. three times each.

Warm-up first, then the median of --reps (>= 20) measurements; one JSON line per measurement.

    python scripts/train_feed_timing.py [--reps 20] [--steps 30] [--augment | --plain-only [--tree DIR]] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--augment", action="store_true", help="time the DATA_AUGMENTOR cases instead of (a)-(c)")
    ap.add_argument("--plain-only", action="store_true", help="time the un-augmented feeder alone instead of (a)-(c)")
    ap.add_argument("--tree", default=None, help="import ptt_amd from this checkout (with --plain-only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.tree:
        if not args.plain_only:
            ap.error("--tree goes with --plain-only")
        sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    from ptt_amd import synth
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.datasets.kitti import kitti_tracking_utils as K
    from ptt_amd.models import build_network
    from ptt_amd.train_feed import TrainBatchFeeder
    from ptt_amd.train_step import DataParallelTrainer, synthetic_train_batch
    dev = torch.device("cuda:0")
    B, reps = args.batch, max(20, args.reps)
    rows = []

    def report(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    tracklets = [synth.tracklet(7000 + k, 12, n_obj=(100, 700), n_bg=(8000, 20000)) for k in range(16)]
    if args.augment:
        augment_cases(tracklets, dev, B, reps, report)
        return save(args.out, rows)
    if args.plain_only:
        plain_only(tracklets, dev, B, reps, report, os.path.abspath(args.tree or HERE))
        return save(args.out, rows)
    feeder = TrainBatchFeeder(tracklets, dev, batch_size=B, seed=1)
    n = len(feeder)

    # (a) the feeder alone
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    feeder.timing_events = (ev0, ev1)
    dev_ms, host_ms, plan_ms = [], [], []
    for k in range(5 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        feeder.batch(0, k % n)
        t1 = time.perf_counter()
        ev1.synchronize()
        t2 = time.perf_counter()
        feeder.plan(0, k % n)
        t3 = time.perf_counter()
        if k >= 5:
            dev_ms.append(ev0.elapsed_time(ev1)), host_ms.append((t1 - t0) * 1e3), plan_ms.append((t3 - t2) * 1e3)
    feeder.timing_events = None
    report(what="a_feeder_alone", batch=B, candidates=feeder.C, largest_cloud=feeder.cap, device_ms=float(np.median(dev_ms)),
           host_ms=float(np.median(host_ms)), host_plan_ms=float(np.median(plan_ms)), **feeder.stats())

    # (b) the per-sample path: one crop_center_pc + get_model + two regularize_pc per sample, each reading its counts back
    pcs = [[K.PointCloud(c) for c in clouds] for clouds, _ in tracklets]
    box = lambda b: K.Box(b[0], b[1], K.Quaternion(array=b[2]))
    per_sample = []
    for k in range(2 + reps):
        plan = feeder.plan(0, k % n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in range(B):
            t, i = int(plan['tracklet'][c]), int(plan['frame'][c])
            gts = tracklets[t][1]
            off_s, off_t = plan['search_offset'][c].copy(), plan['template_offset'][c].copy()
            sample_box = K.get_box_by_offset(box(gts[i]), off_s, True)
            pc, label, reg = K.crop_center_pc(pcs[t][i], sample_box, box(gts[i]), off_s, 0.0, 1.25)
            if pc.nbr_points() > 20:
                K.regularize_pc(pc, 1024, label=label, reg=reg)
            p = max(i - 1, 0)
            model = K.get_model([pcs[t][0], pcs[t][p]], [box(gts[0]), K.get_box_by_offset(box(gts[p]), off_t, True)], 0.0, 1.25)
            if model.nbr_points() > 20:
                K.regularize_pc(model, 512)
        torch.cuda.synchronize()
        if k >= 2:
            per_sample.append((time.perf_counter() - t0) * 1e3)
    report(what="b_per_sample_functions", batch=B, wall_ms=float(np.median(per_sample)))

    # (c) the graphed step: resident batch, fed on the step's stream, fed from a side stream
    torch.manual_seed(1)
    model = build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev).train()
    trainer = DataParallelTrainer(model, dev, graph=True)
    resident = synthetic_train_batch(100, B, dev)
    side = TrainBatchFeeder(tracklets, dev, batch_size=B, seed=1, stream=torch.cuda.Stream(device=dev))
    for _ in range(6):
        trainer.step(resident)
    torch.cuda.synchronize()
    assert trainer.captured is not None

    def run(source, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            trainer.step(resident if source is None else source.batch(0, k % n))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for name, source in (("c_step_resident", None), ("c_step_fed_same_stream", feeder), ("c_step_fed_side_stream", side)) * 3:
        run(source, 5)
        report(what=name, batch=B, steps=args.steps, step_ms=run(source, args.steps), graph_steps=trainer.graph_steps)
    save(args.out, rows)


def save(out, rows):
    if out:
        with open(out, "w") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


def plain_only(tracklets, dev, B, reps, report, tree):
    import numpy as np
    import torch
    from ptt_amd import _lib
    from ptt_amd.train_feed import TrainBatchFeeder
    assert os.path.abspath(_lib.__file__).startswith(tree + os.sep), (_lib.__file__, tree)
    feeder = TrainBatchFeeder(tracklets, dev, batch_size=B, seed=1)
    n = len(feeder)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    feeder.timing_events = (ev0, ev1)
    ms = []
    for k in range(5 + reps):
        torch.cuda.synchronize()
        feeder.batch(0, k % n)
        ev1.synchronize()
        if k >= 5:
            ms.append(ev0.elapsed_time(ev1))
    report(what="plain_only", tree=tree, abi=_lib.ABI_VERSION, batch=B, candidates=feeder.C, reps=len(ms), device_ms=float(np.median(ms)),
           device_ms_min=float(min(ms)), device_ms_max=float(max(ms)), last_batch_sum=float(feeder.last.search.double().sum().cpu()))


P2B_AUGMENTOR = [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
                 {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.78539816, 0.78539816]}]


def augment_cases(tracklets, dev, B, reps, report):
    import numpy as np
    import torch
    from ptt_amd.train_feed import TrainBatchFeeder, TrainBatchPlan
    plain = TrainBatchFeeder(tracklets, dev, batch_size=B, seed=1)
    augmented = TrainBatchFeeder(tracklets, dev, batch_size=B, seed=1, augmentor=P2B_AUGMENTOR)
    maps_of = TrainBatchPlan(tracklets, batch_size=B, seed=1, augmentor=P2B_AUGMENTOR, rank=plain.rank, world=plain.world)
    n = len(plain)
    pinned = torch.zeros((B, 5), dtype=torch.float32).pin_memory()
    maps_dev = torch.zeros((B, 5), dtype=torch.float32, device=dev)

    def stock_maps(k):                          # the host's part, outside the timed span
        pinned.numpy()[:] = maps_of.plan(0, k % n)['aug_map'][:B]

    def stock_ops(batch):
        maps_dev.copy_(pinned, non_blocking=True)
        M, kz = maps_dev[:, 0:4].view(B, 2, 2).transpose(1, 2), maps_dev[:, 4].view(B, 1)
        for pts in (batch['search_points'], batch['template_points']):
            pts[:, :, 0:2] = torch.bmm(pts[:, :, 0:2], M)
            pts[:, :, 2] *= kz

    cases = (("d_plain", plain, None), ("d_augmented", augmented, None), ("d_plain_plus_stock_ops", plain, stock_ops))
    times = {name: {'device_ms': [], 'host_ms': []} for name, _, _ in cases}
    end = torch.cuda.Event(enable_timing=True)
    for k in range(5 + reps):
        for name, feeder, after in cases:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            feeder.timing_events = (ev0, ev1)
            if after is not None:
                stock_maps(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch = feeder.batch(0, k % n)
            if after is not None:
                after(batch)
            end.record(feeder.stream)
            t1 = time.perf_counter()
            end.synchronize()
            feeder.timing_events = None
            if k >= 5:
                times[name]['device_ms'].append(ev0.elapsed_time(end if after is not None else ev1))
                times[name]['host_ms'].append((t1 - t0) * 1e3)
    for name, feeder, _ in cases:
        d = times[name]['device_ms']
        report(what=name, batch=B, candidates=feeder.C, search_size=feeder.S, template_size=feeder.T, largest_cloud=feeder.cap, reps=len(d),
               device_ms=float(np.median(d)), device_ms_min=float(min(d)), device_ms_max=float(max(d)),
               host_ms=float(np.median(times[name]['host_ms'])))


if __name__ == "__main__":
    main()
