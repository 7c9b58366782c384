"""Command-line tools: `python -m ptt_amd.tools.kitti_eval` evaluates a checkpoint on a KITTI tracking directory."""
