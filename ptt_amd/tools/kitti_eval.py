"""Evaluate a checkpoint on a KITTI tracking directory: Success / Precision of the tracking loop over the split's tracklets.

    python -m ptt_amd.tools.kitti_eval --cfg_file tools/cfgs/kitti_models/ptt.yaml --ckpt checkpoint_epoch_60.pth \
        [--data_path /data/kitti] [--split test] [--slots 48] [--results track_result.txt] [--missing origin|raise]

The config is a reference YAML as ptt_amd.config reads it. The tracklets come from the files (datasets/kitti/kitti_scenes.py:
DATA_CONFIG.DATA_PATH unless --data_path, DATA_SPLIT.test unless --split, REF_COOR, CLASS_NAMES), the loop is
PackedTrackletRunner with TEST.SHAPE_AGGREGATION / TEST.REF_BOX and DATA_CONFIG's sizes and offsets (fit.runner_args), the
scores are eval_metrics.evaluate's under REF_COOR. --results writes every result box as a line of the reference's
track_result file (kitti_files.write_track_results): scene, frame, tracklet number, the 24 corner coordinates.
"""
import argparse
import json
import logging

import torch


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--cfg_file", required=True)
    p.add_argument("--ckpt", required=True)
    p.add_argument("--data_path", default=None)
    p.add_argument("--split", default=None)
    p.add_argument("--slots", type=int, default=48)
    p.add_argument("--results", default=None)
    p.add_argument("--missing", default="origin", choices=("origin", "raise"))
    p.add_argument("--device", default="cuda")
    return p.parse_args(argv)


def evaluate_scenes(model, scenes, data_cfg, test_cfg=None, slots=48, results=None):
    """PackedTrackletRunner over a loaded KittiTrackingScenes -> eval_metrics.evaluate's dict; results: a path for the result lines."""
    from .. import eval_metrics
    from ..datasets.kitti import kitti_files
    from ..fit import runner_args
    from ..packed_runner import PackedTrackletRunner
    device = next(model.parameters()).device
    tracklets = scenes.tracklets(offset=-1)
    runner = PackedTrackletRunner(model, device, slots=slots, **runner_args(data_cfg, test_cfg))
    boxes = runner.run(tracklets)
    if results is not None:
        with open(results, "w") as fp:
            for number, (meta, rows) in enumerate(zip(scenes.meta, boxes)):
                for frame, row in zip(meta["frames"], rows):
                    kitti_files.write_track_results(fp, meta["scene"], frame, number, row[:3])
    return eval_metrics.evaluate(boxes, tracklets, ref_coord=scenes.ref_coor, device=device)


def main(argv=None):
    from ..config import EasyDict, StubDataset, cfg_from_yaml_file
    from ..datasets.kitti.kitti_scenes import KittiTrackingScenes
    from ..models import build_network
    args = parse_args(argv)
    logger = logging.getLogger("kitti_eval")
    cfg = cfg_from_yaml_file(args.cfg_file, EasyDict())
    data_cfg = cfg['DATA_CONFIG']
    names = cfg['CLASS_NAMES'] if 'CLASS_NAMES' in cfg else 'Car'
    names = [names] if isinstance(names, str) else list(names)
    if len(names) != 1:
        raise SystemExit("one class is tracked at a time, CLASS_NAMES = %r" % (names,))
    device = torch.device(args.device)
    model = build_network(cfg['MODEL'], len(names), StubDataset(training=False, class_names=names)).to(device)
    model.load_params_from_file(args.ckpt, logger)
    model.eval()
    scenes = KittiTrackingScenes(args.data_path if args.data_path is not None else data_cfg['DATA_PATH'], class_name=names[0],
                                 split=args.split if args.split is not None else data_cfg['DATA_SPLIT']['test'],
                                 ref_coor=data_cfg['REF_COOR'], device=device, missing=args.missing).load()
    res = evaluate_scenes(model, scenes, data_cfg, cfg['TEST'] if 'TEST' in cfg else None, args.slots, args.results)
    logger.info("scenes %s: %d tracklets, %d frames" % (" ".join(scenes.scenes), len(scenes.meta), int(res["frames"].sum())))
    logger.info("Success %.2f  Precision %.2f" % (res["success"], res["precision"]))
    print(json.dumps({"success": res["success"], "precision": res["precision"], "tracklets": len(scenes.meta),
                      "frames": int(res["frames"].sum())}))
    return res


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    main()
