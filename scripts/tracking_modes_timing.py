"""Dev tool: TrackletRunner's cost per frame in every TEST mode (SHAPE_AGGREGATION x REF_BOX) at B = 1 and B = 48 on 200-frame
synthetic tracklets — runner.profile's device_ms (crop + resample + model + read-back on the device) and frame_ms (the whole
step, host included), medians over the frames of a measured run() after a warm-up run(). For SHAPE_AGGREGATION = all also
the median of the first 20 against the last 20 frames: the store is appended to, never re-cropped, so the cost per frame
should not grow with the frame index.

    python scripts/tracking_modes_timing.py [--parent TREE] [--rounds 2] [--frames 200] [--out FILE]

--parent TREE: a checkout of another commit with its library built (ptt_amd/lib/libptt_hip.so); its default mode and this
tree's are then measured in alternating child processes (TREE, this, TREE, this, ...), one per batch size and round.
Every measurement runs in a fresh child process with a time limit; a failing child ends the script."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("firstandprevious", "previous_result"), ("first", "previous_result"), ("previous", "previous_result"),
         ("all", "previous_result"), ("all", "previous_gt"), ("all", "current_gt"), ("firstandprevious", "current_gt")]


def worker(root, batch, modes, frames):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from ptt_amd import synth
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    from ptt_amd.tracklet_runner import TrackletRunner
    dev = torch.device("cuda:0")
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=0).to(dev).eval()
    with torch.no_grad():                                   # small regression outputs: the boxes stay on their objects
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    tracklets = [synth.tracklet(9000 + k, frames, n_bg=(500, 1500)) for k in range(batch)]
    out = []
    for shape, ref in modes:
        kw = {} if (shape, ref) == ("firstandprevious", "previous_result") else {"shape_aggregation": shape, "ref_box": ref}
        runner = TrackletRunner(tracker, dev, batch=batch, **kw)
        runner.run([(c[:8], b[:8]) for c, b in tracklets])       # capture, weight packing
        runner.profile = {}
        runner.run(tracklets)
        torch.cuda.synchronize()
        p = {k: np.asarray(v) for k, v in runner.profile.items()}
        row = {"root": root, "batch": batch, "shape": shape, "ref": ref, "frames": int(len(p["frame_ms"])),
               "device_ms": float(np.median(p["device_ms"])), "frame_ms": float(np.median(p["frame_ms"]))}
        if shape == "all":
            row.update(first20_device_ms=float(np.median(p["device_ms"][:20])), last20_device_ms=float(np.median(p["device_ms"][-20:])),
                       first20_frame_ms=float(np.median(p["frame_ms"][:20])), last20_frame_ms=float(np.median(p["frame_ms"][-20:])),
                       store_growths=int(runner.store_growths))
        out.append(row)
        print(json.dumps(row), flush=True)
        del runner
    return out


def _child(root, batch, modes, frames, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--batch", str(batch), "--frames", str(frames),
           "--modes", ",".join("%s:%s" % m for m in modes)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=timeout)
    if proc.returncode != 0:
        raise SystemExit("child %s exited with %d" % (" ".join(cmd), proc.returncode))
    rows = [json.loads(l) for l in proc.stdout.decode().splitlines() if l.startswith("{")]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--modes", default="")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batches", default="1,48")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.batch, [tuple(m.split(":")) for m in a.modes.split(",")], a.frames)
        return
    rows = []
    batches = [int(b) for b in a.batches.split(",")]
    for b in batches:
        rows += _child(HERE, b, MODES, a.frames, a.timeout)
    if a.parent:                                             # the default mode, parent and this tree alternating
        for _ in range(a.rounds):
            for b in batches:
                for root in (os.path.abspath(a.parent), HERE):
                    rows += [dict(r, ab=True) for r in _child(root, b, [MODES[0]], a.frames, a.timeout)]
    print("\n%-6s %-18s %-16s %-8s %10s %10s  %s" % ("batch", "shape", "ref", "tree", "device_ms", "frame_ms", "all: first 20 -> last 20 frames (device / frame ms)"))
    for r in rows:
        tree = ("parent" if r["root"] != HERE else "branch") + ("*" if r.get("ab") else "")
        extra = ""
        if "first20_device_ms" in r:
            extra = "%.3f -> %.3f / %.3f -> %.3f (store grew %d x)" % (r["first20_device_ms"], r["last20_device_ms"], r["first20_frame_ms"],
                                                                       r["last20_frame_ms"], r["store_growths"])
        print("%-6d %-18s %-16s %-8s %10.3f %10.3f  %s" % (r["batch"], r["shape"], r["ref"], tree, r["device_ms"], r["frame_ms"], extra))
    print("(* = the alternating default-mode A/B runs)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
